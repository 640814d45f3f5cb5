"""Partitioned indexes (round 5; include/finito_amd.h: fin_pindex_*): a unitig set held as parts, each an ordinary index below 2^32 nodes, must answer
pair for pair what ONE index of all the unitigs answers -- the reference's FinimizerIndex over the whole set (FinimizerIndex.hh:26-259, unitig numbers by
permute_unitigs, PackedStrings.hh:105-135) -- which the oracle computes here; and a set that is not a disjoint spectrum-preserving string set
(README.md:79-80) must be refused.  The sizes here force parts of a few thousand bases; bench.py --parts runs a set beyond 2^32 nodes.

Round 35 adds the contracts around the answers (include/finito_amd.h): a prefix holds ONE index (a save removes the other kind's files), fin_pindex_free and
fin_pbatch_free in either order, the 1024-run window of fin_pbatch_step_time, what an unchecked set returns -- and the edges: k above 128, parts of one unitig, a
set of one unitig, read sets without a k-mer, one batch reloaded across sizes, the set-wide unitig numbers stated directly, the number in verify's refusal.  Every
expectation is the oracle's over the whole set, plain Python over the unitig strings, or the one-index FinimizerIndex answer; none comes from the partitioned code.
Measured on one MI355X: the 1030-run loop of the window test (20 reads of 60 bases, 3 parts) runs in 0.4 s with its index build; no test here takes more than
2.5 s and the module takes 16 s."""
import numpy as np
import pytest

import finito_amd as fa


def _reads(rng, g, k, unitigs):
    from tests.test_search_gpu import _fast_path_reads
    from tests.util import sample_reads
    return _fast_path_reads(rng, g, k, unitigs) + sample_reads(rng, g, 300, 150 if k < 100 else 400, err=0.02) + ["", "ACGT", g[100:100 + k - 1], g[50:50 + k]]


def split_parts(unitigs, max_part):
    """the parts as include/finito_amd.h states them -- consecutive input unitigs while they fit in max_part bases --: [(first input unitig, one past the last)]"""
    cuts, in_part = [0], 0
    for u, s in enumerate(unitigs):
        if in_part + len(s) > max_part:
            cuts.append(u); in_part = 0
        in_part += len(s)
    return list(zip(cuts, cuts[1:] + [len(unitigs)]))


def set_wide_numbers(unitigs, k):
    """per input unitig its number in the set: its rank among ALL unitigs sorted by first k-mer in colex order, ties by input order (sorted() is stable)"""
    order = sorted(range(len(unitigs)), key=lambda u: unitigs[u][:k][::-1])
    num = np.empty(len(unitigs), dtype=np.int64)
    num[order] = np.arange(len(unitigs))
    return num


def split_parts_unchecked(unitigs, k, max_part):
    """the parts of an UNCHECKED set (include/finito_amd.h): split_parts, and a part that holds a k-mer twice (same strand) is cut in front of the first unitig
    that repeats a k-mer of the unitigs before it, the rest looked at in its turn"""
    out = []
    todo = split_parts(unitigs, max_part)
    while todo:
        a, b = todo.pop(0)
        seen = set()
        for u in range(a, b):
            if u > a and any(m in seen for m in kmers_of(unitigs[u].upper(), k)):
                out.append((a, u)); todo.insert(0, (u, b))
                break
            seen.update(kmers_of(unitigs[u].upper(), k))
        else:
            out.append((a, b))
    return out


def assert_set_wide_numbers(p, unitigs, k, max_part, parts=None):
    """the direct statement: every part's table is the set-wide numbers of its unitigs (ascending: a part's own order is the set's, restricted); exact, no search"""
    num = set_wide_numbers(unitigs, k)
    parts = parts or split_parts(unitigs, max_part)
    assert p.n_parts == len(parts)
    for i, (a, b) in enumerate(parts):
        assert np.array_equal(p.unitig_ids(i).astype(np.int64), np.sort(num[a:b])), "part %d of %d" % (i, len(parts))
    return parts


def kmers_of(s, k):
    return [s[i:i + k] for i in range(len(s) - k + 1)]


_CASE = {}


def small_case(k=31):
    """the one input the tests below share (made once per k; nobody changes it): a 40 000-base genome cut into unitigs of at most 700 bases, 300 reads of 150 bases
    with errors plus reads without a k-mer, and the oracle's pairs for them over the whole set"""
    if k not in _CASE:
        from types import SimpleNamespace
        from oracle.oracle import OracleIndex
        from tests.util import cut_unitigs, random_genome, sample_reads
        rng = np.random.default_rng(7700 + k)
        g = random_genome(rng, 40000)
        unitigs = cut_unitigs(rng, g, k, max_len=700)
        reads = sample_reads(rng, g, 300, 150, err=0.02) + ["", "ACGT", g[100:100 + k - 1], g[50:50 + k]]
        o = OracleIndex.build(unitigs, k)
        exp, _, _ = o.search_batch(reads)
        exp.setflags(write=False)
        _CASE[k] = SimpleNamespace(k=k, g=g, unitigs=unitigs, reads=reads, oracle=o, exp=exp, found=int((exp[:, 0] != -1).sum()))
    return _CASE[k]


def _reload(b, reads):
    """fin_pbatch_reload through ctypes (the Python class has no reload): the return code"""
    import ctypes as C
    bases, offsets = fa.flatten(reads)
    err = C.create_string_buffer(512)
    rc = b.L.fin_pbatch_reload(b.h, bases.ctypes.data_as(C.c_char_p), offsets.ctypes.data_as(C.POINTER(C.c_uint64)), len(offsets) - 1, err, 512)
    b.n_kmers = int(b.L.fin_pbatch_n_kmers(b.h))   # (read again: download() sizes its buffer by it)
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("k,max_part", [(31, 9000), (21, 25000), (63, 12000), (47, 100000), (100, 15000), (129, 20000), (200, 20000), (255, 25000)])
def test_parts_answer_as_one_index(k, max_part):
    from oracle.oracle import OracleIndex
    from tests.util import cut_unitigs, random_genome
    rng = np.random.default_rng(1000 + k)
    g = random_genome(rng, 60000)
    unitigs = cut_unitigs(rng, g, k, max_len=900)
    reads = _reads(rng, g, k, unitigs)
    o = OracleIndex.build(unitigs, k)
    exp, _, _ = o.search_batch(reads)
    one = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    want, want_pos = one.search_reads(reads)
    assert np.array_equal(want.astype(np.int64), exp)
    p = fa.PartitionedIndex(unitigs, k, device=0, max_part_bases=max_part, verify=True)
    try:
        total = sum(len(u) for u in unitigs)
        assert (p.n_parts == 1) if max_part >= total else (p.n_parts >= 3 and p.n_parts == len(p.part_nodes()))
        assert p.shared_kmers == 0 and p.n_unitigs == len(unitigs) and p.total_len == total and p.n_kmers == one.n_kmers
        assert p.n_nodes >= one.n_nodes   # (every part brings its own dummy nodes)
        # the set's unitig numbers are permute_unitigs' over ALL unitigs: the parts' tables together are a permutation, each ascending
        ids = np.concatenate([p.unitig_ids(i) for i in range(p.n_parts)])
        assert np.array_equal(np.sort(ids), np.arange(len(unitigs), dtype=np.uint32))
        assert_set_wide_numbers(p, unitigs, k, max_part)
        assert all((np.diff(p.unitig_ids(i).astype(np.int64)) > 0).all() for i in range(p.n_parts))
        got, npos = p.search_reads(reads)
        assert np.array_equal(got.astype(np.int64), exp), "k=%d: parts and the whole index disagree" % k
        assert npos == want_pos == int((exp[:, 0] != -1).sum())
        # the device-resident form, run twice (the first part's buffer is the set's result: a second run must not see renumbered pairs)
        b = p.batch(reads)
        b.run(); b.run()
        got2, npos2 = b.download()
        assert np.array_equal(got2, got) and npos2 == npos
        ms, n = b.step_time_ms()
        assert n == 2 and ms > 0
        b.close()
    finally:
        p.close(); one.close()


@pytest.mark.gpu
def test_a_set_that_is_not_disjoint_is_refused():
    from tests.util import cut_unitigs, random_genome, rc
    rng = np.random.default_rng(4242)
    k = 31
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=700)
    fa.PartitionedIndex(unitigs, k, max_part_bases=8000).close()   # the set itself is fine
    far = len(unitigs) - 1
    long3 = next(u for u in unitigs[:8] if len(u) >= k + 40)
    for extra, where in ((unitigs[0][:200], far), (rc(unitigs[1][:150]), far), (long3[5:5 + k], far), (unitigs[2], 3)):
        # a stretch of an early unitig again -- as it is, reverse-complemented, a single k-mer -- in a part far behind; a whole unitig twice inside one part
        bad = unitigs[:where] + [extra] + unitigs[where:]
        with pytest.raises(fa.FinitoError) as e:
            fa.PartitionedIndex(bad, k, max_part_bases=8000, verify=True)
        assert e.value.code == fa.FIN_EINVAL and "disjoint" in str(e.value)
        q = fa.PartitionedIndex(bad, k, max_part_bases=8000, verify=False)   # unchecked: builds (and is the caller's risk)
        assert q.shared_kmers == -1
        q.close()
    with pytest.raises(fa.FinitoError):
        fa.PartitionedIndex(unitigs + ["ACGT"], k, max_part_bases=8000)   # a unitig shorter than k
    with pytest.raises(fa.FinitoError):
        fa.PartitionedIndex(unitigs, k, max_part_bases=300)               # a unitig longer than a part may be


@pytest.mark.gpu
def test_partitioned_index_on_disk_and_through_the_command(tmp_path):
    """serialize / load (the manifest, every part's container, the tables of set-wide unitig numbers) and the command: `finito build-fmin --parts-max-bases`
    writes a partitioned index, `finito search-fmin` finds it by its manifest and prints the text the one-index run prints, byte for byte
    (search_fmin.hh:62-65 through the host formatter)"""
    import os
    import subprocess
    from tests.util import cut_unitigs, random_genome
    rng = np.random.default_rng(909)
    k = 31
    g = random_genome(rng, 50000)
    unitigs = cut_unitigs(rng, g, k, max_len=800)
    reads = _reads(rng, g, k, unitigs)
    reads = [r for r in reads if len(r) > 0]   # (FASTA records)
    p = fa.PartitionedIndex(unitigs, k, max_part_bases=12000)
    want, want_pos = p.search_reads(reads)
    p.serialize(str(tmp_path / "px"))
    assert fa.PartitionedIndex.exists(str(tmp_path / "px")) and not fa.PartitionedIndex.exists(str(tmp_path / "nothing"))
    n_parts = p.n_parts
    p.close()
    q = fa.PartitionedIndex.load(str(tmp_path / "px"))
    assert q.n_parts == n_parts and q.k == k and q.n_unitigs == len(unitigs) and q.shared_kmers == 0
    got, got_pos = q.search_reads(reads)
    assert np.array_equal(got, want) and got_pos == want_pos
    got2, _ = q.search_reads(reads[:100])   # (the set's cached device batches, reloaded with another read set)
    assert np.array_equal(got2, want[: len(got2)])
    q.close()
    with open(tmp_path / "px.p1.gid", "r+b") as f:   # a damaged table is refused
        f.truncate(8)
    with pytest.raises(fa.FinitoError):
        fa.PartitionedIndex.load(str(tmp_path / "px"))
    # the command
    cli = os.path.join(os.path.dirname(fa.__file__), "finito")
    ufa, rfa = tmp_path / "u.fna", tmp_path / "r.fna"
    ufa.write_text("".join(">u%d\n%s\n" % (i, u) for i, u in enumerate(unitigs)))
    rfa.write_text("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    for tag, extra in (("one", []), ("parts", ["--parts-max-bases", "12000"])):
        b = subprocess.run([cli, "build-fmin", "-u", str(ufa), "-o", str(tmp_path / tag), "-k", str(k)] + extra, capture_output=True, text=True, timeout=300)
        assert b.returncode == 0, b.stderr[-800:]
        sr = subprocess.run([cli, "search-fmin", "-i", str(tmp_path / tag), "-q", str(rfa), "-o", str(tmp_path / (tag + ".txt")), "--gpus", "1"], capture_output=True, text=True, timeout=300)
        assert sr.returncode == 0, sr.stderr[-800:]
    assert os.path.exists(tmp_path / "parts.finparts") and not os.path.exists(tmp_path / "one.finparts")
    a, b_ = open(tmp_path / "one.txt", "rb").read(), open(tmp_path / "parts.txt", "rb").read()
    assert a == b_ and len(a) > 10000
    exp = fa.format_pairs  # (the text of the pairs the API delivered, read by read)
    nk = [max(0, len(r) - k + 1) for r in reads]
    off = np.concatenate([[0], np.cumsum(nk)])
    assert b_ == "".join(exp(want[off[i]:off[i + 1]]) for i in range(len(reads))).encode()


# ---- saving over another kind of index (include/finito_amd.h: saving under a prefix replaces what was there) --------------------------------------------------

@pytest.mark.gpu
def test_a_plain_build_over_a_partitioned_prefix_answers_for_its_own_unitigs(tmp_path):
    """`build-fmin --parts-max-bases` on unitig set A, then a plain `build-fmin` on set B under the same prefix: search-fmin must answer for B -- byte for byte
    what it prints for B under a fresh prefix, which is the oracle's answer for B as text.  (The parent commit left A's manifest and part files in place and
    answered from A, exit status 0.)"""
    import glob
    import os
    import subprocess
    from oracle.oracle import OracleIndex
    from tests.util import cut_unitigs, random_genome, sample_reads
    rng = np.random.default_rng(606)
    k = 31
    gA, gB = random_genome(rng, 40000), random_genome(rng, 40000)
    A, B = cut_unitigs(rng, gA, k, max_len=800), cut_unitigs(rng, gB, k, max_len=800)
    reads = sample_reads(rng, gA, 150, 150, err=0.02) + sample_reads(rng, gB, 150, 150, err=0.02) + ["ACGT", gB[100:100 + k - 1], gB[50:50 + k]]
    expA, _, _ = OracleIndex.build(A, k).search_batch(reads)
    expB, _, _ = OracleIndex.build(B, k).search_batch(reads)
    assert not np.array_equal(expA, expB) and (expA[:, 0] != -1).sum() > 5000 and (expB[:, 0] != -1).sum() > 5000   # (the guard: a stale answer shows)
    cli = os.path.join(os.path.dirname(fa.__file__), "finito")
    fA, fB, rfa = tmp_path / "a.fna", tmp_path / "b.fna", tmp_path / "r.fna"
    fA.write_text("".join(">u%d\n%s\n" % (i, u) for i, u in enumerate(A)))
    fB.write_text("".join(">u%d\n%s\n" % (i, u) for i, u in enumerate(B)))
    rfa.write_text("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))

    def run(*args):
        r = subprocess.run([cli] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-800:]

    P, Q = tmp_path / "P", tmp_path / "Q"
    run("build-fmin", "-u", fA, "-o", P, "-k", k, "--parts-max-bases", 12000)
    assert os.path.exists(str(P) + ".finparts") and len(glob.glob(str(P) + ".p*.finamd")) >= 3
    run("build-fmin", "-u", fB, "-o", P, "-k", k)
    assert not fa.PartitionedIndex.exists(str(P)) and glob.glob(str(P) + ".p*") == []
    run("build-fmin", "-u", fB, "-o", Q, "-k", k)
    run("search-fmin", "-i", P, "-q", rfa, "-o", tmp_path / "P.txt", "--gpus", 1)
    run("search-fmin", "-i", Q, "-q", rfa, "-o", tmp_path / "Q.txt", "--gpus", 1)
    got, fresh = open(tmp_path / "P.txt", "rb").read(), open(tmp_path / "Q.txt", "rb").read()
    off = np.concatenate([[0], np.cumsum([max(0, len(r) - k + 1) for r in reads])])
    assert fresh == "".join(fa.format_pairs(expB[off[i]:off[i + 1]]) for i in range(len(reads))).encode()
    assert got == fresh


@pytest.mark.gpu
def test_a_smaller_partitioned_index_saved_over_a_larger_one(tmp_path):
    """fin_pindex_save of 2 parts under a prefix that holds 5 or more: no part file from 2 up is left (nor a one-index container), and load answers as the oracle
    does for the smaller set"""
    import glob
    import os
    from oracle.oracle import OracleIndex
    c = small_case()
    k = c.k
    pre = str(tmp_path / "px")
    big = fa.PartitionedIndex(c.unitigs, k, max_part_bases=8000)
    assert big.n_parts >= 5
    big.serialize(pre)
    n_big = big.n_parts
    big.close()
    assert sorted(glob.glob(pre + ".p*")) == sorted(pre + ".p%d.%s" % (i, e) for i in range(n_big) for e in ("finamd", "gid"))
    few = c.unitigs[:24]
    total = sum(len(u) for u in few)
    one = fa.FinimizerIndex.build(few, k)
    one.serialize(pre)   # (a one-index save in between: it takes the partitioned index away ...)
    assert glob.glob(pre + ".*") == [pre + ".finamd"]
    with pytest.raises(fa.FinitoError):
        fa.PartitionedIndex.load(pre)
    big = fa.PartitionedIndex(c.unitigs, k, max_part_bases=8000)   # (... and the larger set again)
    big.serialize(pre)
    big.close()
    assert len(glob.glob(pre + ".p*")) == 2 * n_big and not os.path.exists(pre + ".finamd")
    small = fa.PartitionedIndex(few, k, max_part_bases=total // 2 + 700)
    assert small.n_parts == 2
    small.serialize(pre)
    small.close(); one.close()
    assert sorted(glob.glob(pre + ".*")) == sorted([pre + ".finparts"] + [pre + ".p%d.%s" % (i, e) for i in range(2) for e in ("finamd", "gid")])
    exp, _, _ = OracleIndex.build(few, k).search_batch(c.reads)
    q = fa.PartitionedIndex.load(pre)
    assert q.n_parts == 2 and q.n_unitigs == len(few)
    got, npos = q.search_reads(c.reads)
    assert np.array_equal(got.astype(np.int64), exp) and npos == int((exp[:, 0] != -1).sum()) and 0 < npos < c.found
    q.close()


# ---- handle lifetimes (include/finito_amd.h: fin_pindex_free and fin_pbatch_free in either order) ---------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("how", ["close", "close_loaded", "collect"])
def test_a_batch_outlives_its_index(how, tmp_path):
    """p.close() (or the index object collected) BEFORE the batch: the batch runs and downloads as before -- the oracle's pairs -- and is freed last.  The parent
    commit freed the parts under the batch here (its fin_pbatch kept a raw pointer to the set): read from the source, never run."""
    import gc
    import weakref
    c = small_case()
    p = fa.PartitionedIndex(c.unitigs, c.k, max_part_bases=8000)
    if how == "close_loaded":
        p.serialize(str(tmp_path / "px"))
        p.close()
        p = fa.PartitionedIndex.load(str(tmp_path / "px"))
    assert p.n_parts >= 3
    got, npos = p.search_reads(c.reads)   # (leaves the set's own cached batch behind: it goes with the owner's reference)
    assert np.array_equal(got.astype(np.int64), c.exp) and npos == c.found
    b = p.batch(c.reads)
    b.run()
    if how == "collect":
        gone = weakref.ref(p)
        del p
        gc.collect()
        assert gone() is None
    else:
        p.close()
        for call in (lambda: p.search_reads(c.reads), lambda: p.batch(c.reads), lambda: p.n_parts, lambda: p.unitig_ids(0), lambda: p.serialize(str(tmp_path / "closed"))):
            with pytest.raises(fa.FinitoError) as e:
                call()
            assert e.value.code == fa.FIN_EINVAL
        p.close()   # (a second close is nothing)
    b.run()
    got2, npos2 = b.download()
    assert np.array_equal(got2.astype(np.int64), c.exp) and npos2 == c.found
    ms, n = b.step_time_ms()
    assert n == 2 and ms > 0
    b.close()


# ---- the timing window ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_step_time_counts_skipped_runs_since_creation_past_the_window():
    """a batch keeps the events of its most recent 1024 runs; after 1030 runs skip_first still counts runs since creation (the parent skipped runs 6 to 15 for
    skip_first = 10, averaging 1014)"""
    import ctypes as C
    c = small_case()
    k = c.k
    reads = [c.g[a:a + 60] for a in range(500, 500 + 20 * 1500, 1500)]
    exp, _, _ = c.oracle.search_batch(reads)
    p = fa.PartitionedIndex(c.unitigs, k, max_part_bases=16000)
    assert p.n_parts in (2, 3)
    b = p.batch(reads)
    err = C.create_string_buffer(512)
    done = 0
    for _ in range(1030):
        if b.L.fin_pbatch_run(b.h, None, err, 512) != 0:
            break
        done += 1
    assert done == 1030, err.value
    got, npos = b.download()
    assert np.array_equal(got.astype(np.int64), exp) and npos == int((exp[:, 0] != -1).sum()) == 20 * (60 - k + 1)
    t0, t6, t10, t_all = b.step_time_ms(0), b.step_time_ms(6), b.step_time_ms(10), b.step_time_ms(1030)
    print("step_time_ms after 1030 runs: skip 0 %r, skip 6 %r, skip 10 %r, skip 1030 %r" % (t0, t6, t10, t_all))
    assert t0[1] == 1024 and t0[0] > 0
    assert t10[1] == 1020 and t10[0] > 0
    assert t6[1] == 1024 and t6[0] > 0
    assert t_all == (0.0, 0)
    b.close(); p.close()


# ---- edges, against the oracle ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["longest_unitig", "one_unitig", "whole_set"])
def test_degenerate_partitions_answer_as_the_oracle(shape):
    """max_part_bases = the longest unitig's length (many parts of one or two unitigs, at least one of exactly one); a set of one unitig; max_part_bases = the
    total (one part)"""
    from oracle.oracle import OracleIndex
    c = small_case()
    k = c.k
    if shape == "one_unitig":
        unitigs = [c.g[3000:3900]]
        max_part = 0
        exp, _, _ = OracleIndex.build(unitigs, k).search_batch(c.reads)
    else:
        unitigs = c.unitigs[:40] if shape == "longest_unitig" else c.unitigs
        max_part = max(len(u) for u in unitigs) if shape == "longest_unitig" else sum(len(u) for u in unitigs)
        exp = c.exp if unitigs is c.unitigs else OracleIndex.build(unitigs, k).search_batch(c.reads)[0]
    p = fa.PartitionedIndex(unitigs, k, max_part_bases=max_part, verify=True)
    try:
        parts = assert_set_wide_numbers(p, unitigs, k, max_part or 10 ** 10)
        if shape == "longest_unitig":
            sizes = [b - a for a, b in parts]
            assert len(parts) >= 15 and 1 in sizes and sizes == [len(p.unitig_ids(i)) for i in range(p.n_parts)]
        else:
            assert p.n_parts == 1
        assert p.shared_kmers == 0 and p.n_unitigs == len(unitigs) and p.total_len == sum(len(u) for u in unitigs)
        got, npos = p.search_reads(c.reads)
        assert np.array_equal(got.astype(np.int64), exp) and npos == int((exp[:, 0] != -1).sum()) > 0
        b = p.batch(c.reads)
        b.run()
        got2, npos2 = b.download()
        assert np.array_equal(got2, got) and npos2 == npos
        b.close()
    finally:
        p.close()


def _outcome(f):
    try:
        pairs, npos = f()
    except fa.FinitoError as e:
        return ("refused", e.code)
    return ("answered", tuple(pairs.shape), npos)


@pytest.mark.gpu
def test_read_sets_without_a_kmer_as_the_one_index():
    """reads = [] and reads that are all shorter than k, through search_reads and through batch / run / download: whatever the one-index FinimizerIndex does with
    them -- an empty result with no k-mer found, or a refusal with its code -- the partitioned index does too; and both still answer afterwards"""
    c = small_case()
    k = c.k
    one = fa.FinimizerIndex.build(c.unitigs, k).to_device(0)
    p = fa.PartitionedIndex(c.unitigs, k, max_part_bases=9000)

    def through_batch(x, reads):
        b = x.batch(reads)
        try:
            b.run()
            return b.download()
        finally:
            b.close()

    try:
        for reads in ([], ["", "ACGT", c.g[100:100 + k - 1]], [""], [c.g[7:7 + k - 1]] * 70):
            want = _outcome(lambda: one.search_reads(reads))
            assert want[0] == "refused" or want == ("answered", (0, 2), 0), want
            assert _outcome(lambda: p.search_reads(reads)) == want, reads[:3]
            want_b = _outcome(lambda: through_batch(one, reads))
            assert want_b[0] == "refused" or want_b == ("answered", (0, 2), 0), want_b
            assert _outcome(lambda: through_batch(p, reads)) == want_b, reads[:3]
        got, npos = p.search_reads(c.reads)   # (the set's cached batch, reloaded from nothing)
        assert np.array_equal(got.astype(np.int64), c.exp) and npos == c.found
    finally:
        p.close(); one.close()


@pytest.mark.gpu
def test_one_batch_reloaded_across_sizes():
    """fin_pbatch_reload: about 50 reads, about 600 (more than at creation), 50, 600 -- after every run the oracle's pairs for that read set, n_kmers read again;
    and a download between a reload and its first run is refused (nothing has run on these reads)"""
    import ctypes as C
    from tests.util import sample_reads
    c = small_case()
    k = c.k
    rng = np.random.default_rng(31337)
    sets = [sample_reads(rng, c.g, n, 150, err=0.02) + ["ACGT", ""] for n in (50, 600, 47, 613)]
    exps = [c.oracle.search_batch(r)[0] for r in sets]
    p = fa.PartitionedIndex(c.unitigs, k, max_part_bases=9000)
    assert p.n_parts >= 3
    b = p.batch(c.reads)   # (created with 304 reads)
    b.run()
    assert np.array_equal(b.download()[0].astype(np.int64), c.exp)
    err = C.create_string_buffer(512)
    try:
        for reads, exp in zip(sets, exps):
            assert _reload(b, reads) == 0
            assert b.n_kmers == len(exp) == sum(max(0, len(r) - k + 1) for r in reads)
            out = np.empty((b.n_kmers, 2), dtype=np.int32)
            assert b.L.fin_pbatch_download(b.h, out.ctypes.data_as(C.c_void_p), None, err, 512) == fa.FIN_EINVAL   # before the first run after a reload
            with pytest.raises(fa.FinitoError) as e:
                b.download()
            assert e.value.code == fa.FIN_EINVAL
            b.run()
            got, npos = b.download()
            assert np.array_equal(got.astype(np.int64), exp) and npos == int((exp[:, 0] != -1).sum()), len(reads)
    finally:
        b.close(); p.close()


_NON_DISJOINT = {}


def non_disjoint_sets(k):
    """(the genome, [(name, unitigs, max_part_bases, reads drawn across the duplicated stretches)]: the four constructions of test_a_set_that_is_not_disjoint_is_refused -- a
    stretch of an early unitig again in a part far behind, as it is / reverse-complemented / a single k-mer; a whole unitig twice inside one part -- and a k-mer
    shared only between the last two parts.  (k = 30 adds a self-reverse-complement k-mer planted in two parts: see the test.)"""
    from tests.util import cut_unitigs, random_genome, rc
    if k in _NON_DISJOINT:
        return _NON_DISJOINT[k]
    rng = np.random.default_rng(4242 + k)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=700)
    far = len(unitigs) - 1
    long3 = next(u for u in unitigs[:8] if len(u) >= k + 40)
    out = []
    for name, extra, where in (("stretch", unitigs[0][:200], far), ("rc_stretch", rc(unitigs[1][:150]), far), ("one_kmer", long3[5:5 + k], far),
                               ("twice_in_a_part", unitigs[2], 3)):
        out.append((name, unitigs[:where] + [extra] + unitigs[where:], extra))
    parts = split_parts(unitigs, 8000)
    a, b = parts[-2]
    src = next(u for u in unitigs[a:b] if len(u) >= k + 60)
    out.append(("last_two_parts", unitigs + [src[20:20 + k + 30]], src[20:20 + k + 30]))
    if k % 2 == 0:
        w = random_genome(rng, k // 2)
        x, y = random_genome(rng, 40) + w + rc(w) + random_genome(rng, 33), random_genome(rng, 29) + w + rc(w) + random_genome(rng, 51)
        assert w + rc(w) == rc(w + rc(w))
        out.append(("self_rc_kmer", [x] + unitigs + [y], w + rc(w)))
    _NON_DISJOINT[k] = (g, out)
    return _NON_DISJOINT[k]


def brute_shared(unitigs, k, parts):
    """what verify counts, in plain Python: over ordered part pairs p < t, the k-mer positions of part p's unitigs whose k-mer or its reverse complement occurs in
    part t; plus, for a part that holds a k-mer more than once, its positions beyond the distinct k-mers (0 for the sets whose parts are disjoint by themselves)"""
    from tests.util import rc
    sets = [{m for u in unitigs[a:b] for m in kmers_of(u, k)} for a, b in parts]
    both = [s | {rc(m) for m in s} for s in sets]
    n = 0
    for pi, (a, b) in enumerate(parts):
        positions = [m for u in unitigs[a:b] for m in kmers_of(u, k)]
        n += len(positions) - len(sets[pi])
        for t in range(pi + 1, len(parts)):
            n += sum(m in both[t] for m in positions)
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("k,name", [(31, "stretch"), (31, "rc_stretch"), (31, "one_kmer"), (31, "twice_in_a_part"), (31, "last_two_parts"), (30, "self_rc_kmer")])
def test_unchecked_sets_and_the_count_of_the_refusal(k, name):
    """Over an input that is NOT disjoint: verify=True refuses with the number of shared occurrences, which is the brute-force count over the unitig strings;
    verify=False builds, and (include/finito_amd.h) every pair it reports is a true occurrence -- the unitig with that set-wide number holds the read's k-mer or
    its reverse complement at that offset -- and a slot is (-1,-1) iff neither occurs anywhere in the set.  Checked with a plain Python set of k-mers.

    "twice_in_a_part" (a whole unitig twice inside ONE part): one index of such a part answers as the reference does over duplicated unitigs -- measured here
    before the build split such parts: five slots of one read came back as (63,4) .. (63,0), places that do not spell k-mers that occur nowhere in the set,
    and the CPU oracle over that part alone gave the same pairs (tests/util.py: DEFER_KAT; common.hh:61-67).  An unchecked build therefore cuts a part in front
    of the first unitig that repeats a k-mer of the unitigs before it (split_parts_unchecked restates the rule), and both properties hold for all six."""
    import re
    from tests.util import rc, sample_reads
    g, cases = non_disjoint_sets(k)
    rng = np.random.default_rng(99 + k)
    common = sample_reads(rng, g, 120, 120, err=0.02)
    for _, bad, dup in (x for x in cases if x[0] == name):
        parts = split_parts(bad, 8000)
        per_part = [{m for u in bad[a:b] for m in kmers_of(u, k)} for a, b in parts]
        disjoint_parts = all(len(s) == sum(len(u) - k + 1 for u in bad[a:b]) for s, (a, b) in zip(per_part, parts))
        assert disjoint_parts == (name != "twice_in_a_part"), name
        want_n = brute_shared(bad, k, parts)
        assert want_n >= 1
        if name == "last_two_parts":   # (the guard: the shared k-mers lie in the last two parts and nowhere else)
            where = [i for i, s in enumerate(per_part) if dup[:k] in s]
            assert where == [len(parts) - 2, len(parts) - 1], where
        if name == "self_rc_kmer":
            assert want_n == 1
        with pytest.raises(fa.FinitoError) as e:
            fa.PartitionedIndex(bad, k, max_part_bases=8000, verify=True)
        assert e.value.code == fa.FIN_EINVAL and "disjoint" in str(e.value)
        m = re.search(r"index set: (\d+) k-mer occurrence\(s\)", str(e.value))
        assert m and int(m.group(1)) == want_n, (name, str(e.value), want_n)
        # unchecked
        reads = common + [dup, rc(dup)]
        for u in bad:   # reads drawn across the duplicated stretch: it, with what lies around it in every unitig that holds its first k-mer, either strand
            for probe in (dup[:k], rc(dup[:k])):
                at = u.find(probe)
                if at >= 0:
                    reads += [u[max(0, at - 40):at + len(dup) + 40], rc(u[max(0, at - 25):at + k + 25])]
        uparts = split_parts_unchecked(bad, k, 8000)   # (an unchecked set's parts: each disjoint by itself)
        uper_part = [{m for u in bad[a:b] for m in kmers_of(u, k)} for a, b in uparts]
        assert all(len(s) == sum(len(u) - k + 1 for u in bad[a:b]) for s, (a, b) in zip(uper_part, uparts))
        assert len(uparts) == len(parts) + (name == "twice_in_a_part")
        q = fa.PartitionedIndex(bad, k, max_part_bases=8000, verify=False)
        try:
            assert q.shared_kmers == -1
            assert_set_wide_numbers(q, bad, k, 8000, parts=uparts)
            got, npos = q.search_reads(reads)
        finally:
            q.close()
        num = set_wide_numbers(bad, k)
        by_number = [None] * len(bad)
        for u, n_ in enumerate(num):
            by_number[n_] = bad[u]
        everything = set().union(*per_part)
        in_two_parts = 0
        slot = 0
        for r in reads:
            for m in kmers_of(r, k):
                u, off = int(got[slot, 0]), int(got[slot, 1])
                slot += 1
                there = m in everything or rc(m) in everything
                if u == -1:
                    assert off == -1 and not there, (name, m)
                else:
                    assert there and 0 <= u < len(bad) and off >= 0 and by_number[u][off:off + k] in (m, rc(m)), (name, m, u, off)
                in_two_parts += sum((m in s or rc(m) in s) for s in uper_part) >= 2
        assert slot == len(got) and npos == int((got[:, 0] != -1).sum())
        assert in_two_parts >= 1, name
