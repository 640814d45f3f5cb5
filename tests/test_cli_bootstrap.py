"""`finito search-fmin --color-refs LIST --abundance FILE --ab-bootstraps B [--ab-seed S]`: every colour line gains the replicates' mean and standard deviation
and a `bootstraps` line follows.  The new columns are compared with EqClasses.bootstrap over the classes of the --eqclasses file of the same run, refilled into
an accumulator here, at relative 1e-9 -- the %.10g print precision, 5e-10, doubled (the resampled counts do not depend on the fill; the estimates differ by
rounding, far below that).  Without --ab-bootstraps the file has the format it had, line for line the first three columns of the bootstrap run's."""
import numpy as np
import pytest

import finito_amd as fa
from tests.test_abundance import fill
from tests.test_cli_abundance import parse_abundance, run
from tests.test_colors_host import pack
from tests.util import cut_unitigs, random_genome, sample_reads

pytestmark = pytest.mark.gpu


def parse_bootstrap(path, n_colors):
    """(alpha, share, mean, sd, the bootstraps line's fields, the file as it would be without --ab-bootstraps)"""
    lines = open(path).read().splitlines()
    assert len(lines) == n_colors + 4
    cols = [ln.split("\t") for ln in lines[:n_colors]]
    assert [int(c[0]) for c in cols] == list(range(n_colors)) and all(len(c) == 5 for c in cols)
    assert [ln.split("\t")[0] for ln in lines[n_colors:]] == ["unaligned", "iterations", "loglik", "bootstraps"]
    plain = "".join("\t".join(c[:3]) + "\n" for c in cols) + "".join(ln + "\n" for ln in lines[n_colors:n_colors + 3])
    return [np.array([float(c[i]) for c in cols]) for i in (1, 2, 3, 4)] + [lines[-1].split("\t"), plain]


def classes_of(path, n_colors):
    eq_lines = [ln.split("\t") for ln in open(path).read().splitlines()]
    return pack([[int(c) for c in x[2].split(",")] for x in eq_lines], n_colors), np.array([int(x[0]) for x in eq_lines], dtype=np.uint64)


def test_cli_bootstrap(tmp_path):
    k, n_colors = 31, 4
    rng = np.random.default_rng(2760)
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
    with open(tmp_path / "q.fq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    r = run("build-fmin", "-o", str(tmp_path / "idx"), "-u", str(tmp_path / "u.fna"), "-k", str(k))
    assert r.returncode == 0, r.stderr
    common = ("search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq"), "--gpus", "1", "--color-refs", str(tmp_path / "refs.txt"), "--no-text", "1")
    ab = ("--ab-lengths", str(tmp_path / "lens.txt"), "--ab-max-iters", "15", "--ab-tol", "0")
    # the argument errors, reported before any search
    rb = run(*common, "--eqclasses", str(tmp_path / "no.tsv"), "--ab-bootstraps", "5")
    assert rb.returncode == 1 and "--ab-bootstraps is only legal together with --abundance" in rb.stderr and "Loading index" not in rb.stderr, rb.stderr
    for bad in ("0", "4097", "-3", "x"):
        rb = run(*common, "--abundance", str(tmp_path / "no.tsv"), "--ab-bootstraps", bad)
        assert rb.returncode == 1 and "--ab-bootstraps" in rb.stderr and "Loading index" not in rb.stderr, rb.stderr
    rb = run(*common, "--abundance", str(tmp_path / "no.tsv"), "--ab-seed", "3")
    assert rb.returncode == 1 and "--ab-seed" in rb.stderr
    rb = run(*common, "--abundance", str(tmp_path / "no.tsv"), "--ab-bootstraps", "3", "--ab-seed", "-1")
    assert rb.returncode == 1 and "--ab-seed" in rb.stderr
    assert not (tmp_path / "no.tsv").exists()
    # with and without the replicates
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    col = p.colors(n_colors)
    eq = col.eqclasses(64)
    for paired, n_boot, seed in ((False, 20, 12345678901234567890), (True, 1, 0)):
        tag = "p" if paired else "s"
        extra = ("--paired", "1") if paired else ()
        r1 = run(*common, *extra, "--eqclasses", str(tmp_path / (tag + "e.tsv")), "--abundance", str(tmp_path / (tag + "b.tsv")), *ab, "--ab-bootstraps", str(n_boot),
                 *(("--ab-seed", str(seed)) if seed else ()))
        assert r1.returncode == 0, r1.stderr
        r0 = run(*common, *extra, "--abundance", str(tmp_path / (tag + "a.tsv")), *ab)
        assert r0.returncode == 0, r0.stderr
        alpha, share, mean, sd, last, plain = parse_bootstrap(tmp_path / (tag + "b.tsv"), n_colors)
        assert last == ["bootstraps", str(n_boot), "seed", str(seed)]
        parse_abundance(tmp_path / (tag + "a.tsv"), n_colors)               # the format it had: three columns, three closing lines
        assert open(tmp_path / (tag + "a.tsv")).read() == plain
        crows, creads = classes_of(tmp_path / (tag + "e.tsv"), n_colors)
        assert int(creads.sum()) <= (len(reads) // 2 if paired else len(reads)) and len(crows) >= n_colors
        t = fill(eq, crows, creads)
        want = eq.bootstrap(n_boot, seed=seed, lengths=lens, max_iters=15, tol=0.0)
        del t
        assert (np.abs(alpha - want.point.alpha) <= 1e-9 * want.point.alpha).all()
        assert (np.abs(mean - want.mean) <= 1e-9 * want.mean).all() and (np.abs(sd - want.sd) <= 1e-9 * want.sd).all()
        assert (sd > 0).all() if n_boot > 1 else not sd.any()
    eq.close(); col.close(); p.close()
